/*
 * lfq_bamidx.hip -- the .bai of a BAM built on the device (lfq_bam_index_build), over lfq_bamidx.h, which
 * says what a record contributes.  Work proportional to the records runs here, work proportional to the chunks and touched windows
 * on the host (lfq_bai_finish):
 *
 *   lfq_bai_record_kernel   one lane per record: lfq_bai_record() into an LfqBaiRec; the first refused record by an atomic minimum
 *                           on one word, which the host reads before anything else is launched
 *   lfq_bai_part_kernel     per workgroup: how many chunk heads, run heads and mapped records it holds, and its largest window key
 *   lfq_bai_scan_kernel     one wavefront: the exclusive prefix of those over the workgroups (sums and a running maximum)
 *   lfq_bai_emit_kernel     per workgroup again, ballot and prefix count inside a wavefront, the wavefronts' totals through LDS:
 *                           a head writes its chunk's (refID, bin, u) to the slot its rank names, the record in front of the next
 *                           head writes v there; a reference's run likewise, with the mapped counts at both ends; a record that is
 *                           the first to touch a window gets a slot in the interval list, one atomic add per workgroup (intervals
 *                           never overlap, so their order is of no consequence)
 *
 * Device memory: the three offset tables, 32 bytes a record, 48 bytes a workgroup and the three lists, each at most one entry per
 * record -- nothing that grows with references times windows.  Every store of the emit kernel is to a slot below the list's
 * capacity, checked at the store.
 *
 * Host only, below the build: lfq_bam_index_parse / _bytes / _query / _free, lfq_bam_record_chain, lfq_bam_record_cuts.
 */
#include <chrono>

#include "lfq_ctx.h"
#include "lfq_bamidx.h"

#define LFQ_BAI_THREADS 128
#define LFQ_BAI_WAVES (LFQ_BAI_THREADS / 64)

struct LfqBaiPart {
    uint32_t n_chunk, n_run, n_mapped, pad_;
    uint64_t key;
};

struct LfqBaiArgs {
    const uint8_t *body;                /* byte 0 of the caller's body on the device: only [rec_off[0], rec_off[n_recs]) is there */
    const int64_t *rec_off, *data_off, *comp_off;
    int64_t n_recs, n_blocks, file_off;
    int32_t n_ref;
    LfqBaiRec *rec;                     /* [n_recs] */
    LfqBaiPart *part, *pre;             /* [n_parts] a workgroup's own, and what lies in front of it */
    int64_t n_parts;
    unsigned long long *counters;       /* 0: the first refused record; 1 .. 3: chunks, runs, intervals */
    LfqBaiChunk *chunks;
    LfqBaiRun *runs;
    LfqBaiIntv *intvs;
    int64_t max_chunks, max_runs, max_intvs;
};

__global__ __launch_bounds__(LFQ_BAI_THREADS) void lfq_bai_record_kernel(LfqBaiArgs A)
{
    const int64_t j = (int64_t)blockIdx.x * LFQ_BAI_THREADS + threadIdx.x;
    if (j >= A.n_recs) {
        return;
    }
    LfqBaiRec R;
    if (!lfq_bai_record(A.body, A.rec_off, j, A.n_ref, A.data_off, A.comp_off, A.n_blocks, A.file_off, &R)) {
        atomicMin(&A.counters[0], (unsigned long long)j);
    }
    A.rec[j] = R;
}

struct LfqBaiLane {                     /* what record j counts for */
    bool chunk_head, run_head, mapped;
    uint64_t key;
};

__device__ __forceinline__ LfqBaiLane bai_lane(const LfqBaiArgs &A, int64_t j)
{
    LfqBaiLane L = {false, false, false, 0};
    if (j < A.n_recs) {
        L.chunk_head = lfq_bai_chunk_head(A.rec, j);
        L.run_head = lfq_bai_run_head(A.rec, j);
        L.mapped = A.rec[j].ref_id >= 0 && A.rec[j].mapped;
        L.key = lfq_bai_key(A.rec[j]);
    }
    return L;
}

/* the inclusive running maximum over the lanes of a wavefront */
__device__ __forceinline__ uint64_t bai_wave_max(uint64_t x, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t y = (uint64_t)__shfl_up((unsigned long long)x, d, 64);
        if (lane >= d && y > x) {
            x = y;
        }
    }
    return x;
}

__device__ __forceinline__ uint32_t bai_wave_sum(uint32_t x, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)x, d, 64);
        if (lane >= d) {
            x += y;
        }
    }
    return x;
}

__global__ __launch_bounds__(LFQ_BAI_THREADS) void lfq_bai_part_kernel(LfqBaiArgs A)
{
    __shared__ uint32_t s_cnt[3][LFQ_BAI_WAVES];
    __shared__ uint64_t s_key[LFQ_BAI_WAVES];
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const LfqBaiLane L = bai_lane(A, (int64_t)blockIdx.x * LFQ_BAI_THREADS + threadIdx.x);
    const uint64_t bc = __ballot(L.chunk_head), br = __ballot(L.run_head), bm = __ballot(L.mapped);
    const uint64_t key = bai_wave_max(L.key, lane);
    if (lane == 63) {
        s_cnt[0][wave] = (uint32_t)__popcll(bc);
        s_cnt[1][wave] = (uint32_t)__popcll(br);
        s_cnt[2][wave] = (uint32_t)__popcll(bm);
        s_key[wave] = key;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        LfqBaiPart P = {0, 0, 0, 0, 0};
        for (int w = 0; w < LFQ_BAI_WAVES; w++) {
            P.n_chunk += s_cnt[0][w];
            P.n_run += s_cnt[1][w];
            P.n_mapped += s_cnt[2][w];
            P.key = s_key[w] > P.key ? s_key[w] : P.key;
        }
        A.part[blockIdx.x] = P;
    }
}

/* one wavefront walks the workgroups' parts 64 at a time and carries the totals */
__global__ __launch_bounds__(64) void lfq_bai_scan_kernel(LfqBaiArgs A)
{
    const int lane = (int)threadIdx.x;
    LfqBaiPart carry = {0, 0, 0, 0, 0};
    for (int64_t base = 0; base < A.n_parts; base += 64) {
        const int64_t i = base + lane;
        LfqBaiPart P = {0, 0, 0, 0, 0};
        if (i < A.n_parts) {
            P = A.part[i];
        }
        const uint32_t ic = bai_wave_sum(P.n_chunk, lane), ir = bai_wave_sum(P.n_run, lane), im = bai_wave_sum(P.n_mapped, lane);
        const uint64_t ik = bai_wave_max(P.key, lane);
        uint64_t ek = (uint64_t)__shfl_up((unsigned long long)ik, 1, 64);
        ek = lane == 0 ? 0 : ek;
        if (i < A.n_parts) {
            LfqBaiPart E;
            E.n_chunk = carry.n_chunk + ic - P.n_chunk;
            E.n_run = carry.n_run + ir - P.n_run;
            E.n_mapped = carry.n_mapped + im - P.n_mapped;
            E.pad_ = 0;
            E.key = ek > carry.key ? ek : carry.key;
            A.pre[i] = E;
        }
        carry.n_chunk += (uint32_t)__shfl((int)ic, 63, 64);
        carry.n_run += (uint32_t)__shfl((int)ir, 63, 64);
        carry.n_mapped += (uint32_t)__shfl((int)im, 63, 64);
        const uint64_t last = (uint64_t)__shfl((unsigned long long)ik, 63, 64);
        carry.key = last > carry.key ? last : carry.key;
    }
    if (lane == 0) {
        A.counters[1] = carry.n_chunk;
        A.counters[2] = carry.n_run;
    }
}

__global__ __launch_bounds__(LFQ_BAI_THREADS) void lfq_bai_emit_kernel(LfqBaiArgs A)
{
    __shared__ uint32_t s_cnt[4][LFQ_BAI_WAVES];
    __shared__ uint64_t s_key[LFQ_BAI_WAVES];
    __shared__ unsigned long long s_base;
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const int64_t j = (int64_t)blockIdx.x * LFQ_BAI_THREADS + threadIdx.x;
    const bool in = j < A.n_recs;
    const LfqBaiLane L = bai_lane(A, j);
    const LfqBaiPart pre = A.pre[blockIdx.x];
    const uint64_t below = (1ull << lane) - 1ull;
    const uint64_t bc = __ballot(L.chunk_head), br = __ballot(L.run_head), bm = __ballot(L.mapped);
    const uint64_t ik = bai_wave_max(L.key, lane);
    uint64_t ek = (uint64_t)__shfl_up((unsigned long long)ik, 1, 64);
    ek = lane == 0 ? 0 : ek;
    if (lane == 63) {
        s_cnt[0][wave] = (uint32_t)__popcll(bc);
        s_cnt[1][wave] = (uint32_t)__popcll(br);
        s_cnt[2][wave] = (uint32_t)__popcll(bm);
        s_key[wave] = ik;
    }
    __syncthreads();
    /* exclusive counts and the maximum in front of this record, over the whole input */
    uint64_t n_chunk = pre.n_chunk + (uint64_t)__popcll(bc & below), n_run = pre.n_run + (uint64_t)__popcll(br & below),
             n_mapped = pre.n_mapped + (uint64_t)__popcll(bm & below), key = ek > pre.key ? ek : pre.key;
    for (int w = 0; w < wave; w++) {
        n_chunk += s_cnt[0][w];
        n_run += s_cnt[1][w];
        n_mapped += s_cnt[2][w];
        key = s_key[w] > key ? s_key[w] : key;
    }
    LfqBaiRec R;
    int32_t w_first = 0;
    bool touches = false;
    if (in) {
        R = A.rec[j];
        if (lfq_bai_in_linear(R)) {
            w_first = lfq_bai_first_window(R, key);
            touches = w_first <= R.w1;
        }
    }
    const uint64_t bt = __ballot(touches);
    if (lane == 63) {
        s_cnt[3][wave] = (uint32_t)__popcll(bt);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t total = 0;
        for (int w = 0; w < LFQ_BAI_WAVES; w++) {
            total += s_cnt[3][w];
        }
        s_base = total ? atomicAdd(&A.counters[3], (unsigned long long)total) : 0ull;
    }
    __syncthreads();
    if (!in) {
        return;
    }
    if (L.chunk_head && (int64_t)n_chunk < A.max_chunks) {
        LfqBaiChunk *c = &A.chunks[n_chunk];
        c->u = R.u;
        c->ref_id = R.ref_id;
        c->bin = R.bin;
    }
    const uint64_t chunks_through = n_chunk + (L.chunk_head ? 1 : 0), runs_through = n_run + (L.run_head ? 1 : 0);
    if (lfq_bai_chunk_tail(A.rec, j, A.n_recs) && chunks_through >= 1 && (int64_t)chunks_through <= A.max_chunks) {
        A.chunks[chunks_through - 1].v = R.v;
    }
    if (L.run_head && (int64_t)n_run < A.max_runs) {
        LfqBaiRun *r = &A.runs[n_run];
        r->u = R.u;
        r->first = j;
        r->mapped_before = (int64_t)n_mapped;
        r->ref_id = R.ref_id;
        r->pad_ = 0;
    }
    if (lfq_bai_run_tail(A.rec, j, A.n_recs) && runs_through >= 1 && (int64_t)runs_through <= A.max_runs) {
        LfqBaiRun *r = &A.runs[runs_through - 1];
        r->v = R.v;
        r->last = j;
        r->mapped_through = (int64_t)n_mapped + (L.mapped ? 1 : 0);
    }
    if (touches) {
        uint64_t at = s_base + (uint64_t)__popcll(bt & below);
        for (int w = 0; w < wave; w++) {
            at += s_cnt[3][w];
        }
        if ((int64_t)at < A.max_intvs) {
            LfqBaiIntv T = {R.u, R.ref_id, w_first, R.w1, 0};
            A.intvs[at] = T;
        }
    }
}

/* ---- host side ------------------------------------------------------------------------------------------------------------------- */
struct LfqBamIdxState {
    uint8_t *d_in = nullptr;            /* the records, when they are not on the device already (grow-only, as all of these) */
    int64_t d_in_bytes = 0;
    uint8_t *d_buf = nullptr;           /* offset tables | records' LfqBaiRec | parts | counters | chunks | runs | intervals */
    int64_t d_bytes = 0;
    uint8_t *h_stage = nullptr;         /* pinned staging of a body that comes in pageable memory */
    int64_t h_stage_bytes = 0;
    uint8_t *h_out = nullptr;           /* the three lists on the host, pinned */
    int64_t h_out_bytes = 0;
    lfq_bam_index_times times = {};
    lfq_vcf_index_times vcf_times = {}; /* of lfq_vcf_index_build (lfq_tbx.hip), which compacts in these buffers */
    LfqBaiArgs lay = {};                /* what lfq_bai_reserve laid out in d_buf: the compaction's part of the kernels' arguments */
    LfqEvPair up_t = {}, kern_t = {}, down_t = {};
};

static LfqBamIdxState *bam_idx_state(lfq_ctx *c)
{
    if (!c->bamidx) {
        c->bamidx = new LfqBamIdxState();
    }
    return c->bamidx;
}

void lfq_bam_index_release(lfq_ctx *c)
{
    if (LfqBamIdxState *S = c->bamidx) {
        if (S->d_in) (void)hipFree(S->d_in);
        if (S->d_buf) (void)hipFree(S->d_buf);
        free_pinned(&S->h_stage, &S->h_stage_bytes);
        free_pinned(&S->h_out, &S->h_out_bytes);
        for (LfqEvPair *t : {&S->up_t, &S->kern_t, &S->down_t}) {
            t->destroy();
        }
        delete S;
        c->bamidx = nullptr;
    }
}

static int bam_idx_add_ms(const LfqEvPair &t, double *acc)
{
    double ms = 0.0;
    LFQ_TRY(t.ms(&ms));
    *acc += ms;
    return LFQ_OK;
}

/* ---- the compaction both index builders run (lfq_ctx.h): lfq_bam_index_build below, lfq_vcf_index_build in lfq_tbx.hip ---------------
 * reserve: d_buf = head_bytes of the caller's own | n_recs LfqBaiRec | parts | counters | chunks | runs | intervals.  The caller's
 * record pass fills rec[] and sets the four counters (0: its own, 1 .. 3: zero) in front of lfq_bai_compact, which launches
 * part / scan / emit on the context's stream and brings the three lists to pinned host memory: valid until the next reserve. */
int lfq_bai_reserve(lfq_ctx *c, int64_t head_bytes, int64_t n_recs, int64_t max_runs, LfqBaiDev *out)
{
    LfqBamIdxState *S = bam_idx_state(c);
    const int64_t n_parts = (n_recs + LFQ_BAI_THREADS - 1) / LFQ_BAI_THREADS;
    const int64_t o_rec = lfq_al(head_bytes), o_part = o_rec + lfq_al(n_recs * (int64_t)sizeof(LfqBaiRec)),
                  o_pre = o_part + lfq_al(n_parts * (int64_t)sizeof(LfqBaiPart)),
                  o_cnt = o_pre + lfq_al(n_parts * (int64_t)sizeof(LfqBaiPart)), o_chunks = o_cnt + lfq_al(64),
                  o_runs = o_chunks + lfq_al(n_recs * (int64_t)sizeof(LfqBaiChunk)),
                  o_intvs = o_runs + lfq_al(max_runs * (int64_t)sizeof(LfqBaiRun)),
                  total = o_intvs + lfq_al(n_recs * (int64_t)sizeof(LfqBaiIntv));
    LFQ_TRY(grow(&S->d_buf, &S->d_bytes, total));
    LfqBaiArgs A;
    memset(&A, 0, sizeof(A));
    A.n_recs = n_recs;
    A.rec = (LfqBaiRec *)(S->d_buf + o_rec);
    A.part = (LfqBaiPart *)(S->d_buf + o_part);
    A.pre = (LfqBaiPart *)(S->d_buf + o_pre);
    A.n_parts = n_parts;
    A.counters = (unsigned long long *)(S->d_buf + o_cnt);
    A.chunks = (LfqBaiChunk *)(S->d_buf + o_chunks);
    A.runs = (LfqBaiRun *)(S->d_buf + o_runs);
    A.intvs = (LfqBaiIntv *)(S->d_buf + o_intvs);
    A.max_chunks = n_recs;
    A.max_runs = max_runs;
    A.max_intvs = n_recs;
    S->lay = A;
    out->head = S->d_buf;
    out->rec = A.rec;
    out->counters = A.counters;
    return LFQ_OK;
}

int lfq_bai_compact(lfq_ctx *c, LfqBaiLists *out)
{
    LfqBamIdxState *S = bam_idx_state(c);
    const LfqBaiArgs &A = S->lay;
    hipStream_t st = c->stream;
    memset(out, 0, sizeof(*out));
    LfqPin<unsigned long long> cnt(c, 4);
    LFQ_PIN_OK(cnt);
    const dim3 grid((unsigned)A.n_parts), block(LFQ_BAI_THREADS);
    LFQ_TRY(S->kern_t.begin(st));
    hipLaunchKernelGGL(lfq_bai_part_kernel, grid, block, 0, st, A);
    LFQ_TRY_HIP(hipGetLastError());
    hipLaunchKernelGGL(lfq_bai_scan_kernel, dim3(1), dim3(64), 0, st, A);
    LFQ_TRY_HIP(hipGetLastError());
    hipLaunchKernelGGL(lfq_bai_emit_kernel, grid, block, 0, st, A);
    LFQ_TRY_HIP(hipGetLastError());
    LFQ_TRY(S->kern_t.end(st));
    LFQ_TRY(S->down_t.begin(st));
    LFQ_TRY_HIP(hipMemcpyAsync(cnt.data(), A.counters, 32, hipMemcpyDeviceToHost, st));
    LFQ_TRY(S->down_t.end(st));
    LFQ_TRY_HIP(hipStreamSynchronize(st));
    LFQ_TRY(bam_idx_add_ms(S->kern_t, &out->kernels_ms));
    LFQ_TRY(bam_idx_add_ms(S->down_t, &out->download_ms));
    const int64_t n_chunks = (int64_t)cnt[1], n_runs = (int64_t)cnt[2], n_intvs = (int64_t)cnt[3];
    if (n_chunks > A.max_chunks || n_runs > A.max_runs || n_intvs > A.max_intvs) {
        return LFQ_ERR_HIP;             /* (the kernels disagree with the record pass) */
    }
    const int64_t h_runs = lfq_al(n_chunks * (int64_t)sizeof(LfqBaiChunk)), h_intvs = h_runs + lfq_al(n_runs * (int64_t)sizeof(LfqBaiRun)),
                  h_total = h_intvs + lfq_al(n_intvs * (int64_t)sizeof(LfqBaiIntv));
    if (h_total > S->h_out_bytes) {
        LFQ_TRY(grow_pinned(&S->h_out, &S->h_out_bytes, std::max<int64_t>(h_total + h_total / 4, 1 << 16)));
    }
    LFQ_TRY(S->down_t.begin(st));
    if (n_chunks) {
        LFQ_TRY_HIP(hipMemcpyAsync(S->h_out, A.chunks, (size_t)n_chunks * sizeof(LfqBaiChunk), hipMemcpyDeviceToHost, st));
    }
    if (n_runs) {
        LFQ_TRY_HIP(hipMemcpyAsync(S->h_out + h_runs, A.runs, (size_t)n_runs * sizeof(LfqBaiRun), hipMemcpyDeviceToHost, st));
    }
    if (n_intvs) {
        LFQ_TRY_HIP(hipMemcpyAsync(S->h_out + h_intvs, A.intvs, (size_t)n_intvs * sizeof(LfqBaiIntv), hipMemcpyDeviceToHost, st));
    }
    LFQ_TRY(S->down_t.end(st));
    LFQ_TRY_HIP(hipStreamSynchronize(st));
    LFQ_TRY(bam_idx_add_ms(S->down_t, &out->download_ms));
    out->chunks = (const LfqBaiChunk *)S->h_out;
    out->runs = (const LfqBaiRun *)(S->h_out + h_runs);
    out->intvs = (const LfqBaiIntv *)(S->h_out + h_intvs);
    out->n_chunks = n_chunks;
    out->n_runs = n_runs;
    out->n_intvs = n_intvs;
    return LFQ_OK;
}

lfq_vcf_index_times *lfq_bai_vcf_times(lfq_ctx *c) { return &bam_idx_state(c)->vcf_times; }

extern "C" int lfq_bam_index_build(lfq_ctx *c, const uint8_t *body, int64_t n_bytes, const int64_t *rec_off, int64_t n_recs,
                                   const int64_t *data_off, const int64_t *comp_off, int64_t n_blocks, int64_t file_off, int32_t n_ref,
                                   lfq_bam_index **out)
{
    if (out) *out = nullptr;
    if (!c || !out) {
        return LFQ_ERR_INVALID;
    }
    LfqBamIdxState *S = bam_idx_state(c);
    S->times = {};
    S->times.first_bad_record = -1;     /* (a refused argument is no record's fault) */
    if ((!body && n_recs > 0) || !lfq_bai_check_args(n_bytes, rec_off, n_recs, data_off, comp_off, n_blocks, file_off, n_ref)) {
        return LFQ_ERR_INVALID;
    }
    if (n_recs > INT32_MAX) {
        return LFQ_ERR_CAPACITY;
    }
    S->times.n_recs = n_recs;
    lfq_bam_index *idx = new lfq_bam_index();
    if (n_recs == 0) {
        idx->refs.assign((size_t)n_ref, LfqBaiRef());
        *out = idx;
        return LFQ_OK;
    }
    struct Drop {                       /* the index is the caller's only when the call succeeds */
        lfq_bam_index *p;
        ~Drop() { delete p; }
    } drop = {idx};
    LFQ_TRY_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const int64_t first = rec_off[0], rec_bytes = rec_off[n_recs] - first;
    const uint8_t *d_recs = lfq_bgzf_resident_bytes(c, body + first, rec_bytes);
    if (!d_recs) {
        d_recs = lfq_bam_framed_resident(c, body + first, rec_bytes);
    }
    const int64_t o_doff = lfq_al((n_recs + 1) * 8), o_coff = o_doff + lfq_al((n_blocks + 1) * 8), o_rec = o_coff + lfq_al((n_blocks + 1) * 8);
    LfqBaiDev dev;
    LFQ_TRY(lfq_bai_reserve(c, o_rec, n_recs, std::min<int64_t>(n_recs, n_ref), &dev));
    const int64_t n_tab = (n_recs + 1) + 2 * (n_blocks + 1);
    LfqPin<int64_t> tab(c, (size_t)n_tab);
    LFQ_PIN_OK(tab);
    LfqPin<unsigned long long> cnt(c, 4);
    LFQ_PIN_OK(cnt);
    memcpy(tab.data(), rec_off, (size_t)(n_recs + 1) * 8);
    memcpy(tab.data() + n_recs + 1, data_off, (size_t)(n_blocks + 1) * 8);
    memcpy(tab.data() + n_recs + 1 + n_blocks + 1, comp_off, (size_t)(n_blocks + 1) * 8);
    cnt[0] = ~0ull;
    cnt[1] = cnt[2] = cnt[3] = 0;
    LFQ_TRY(S->up_t.begin(st));
    if (d_recs) {
        S->times.n_from_device = 1;
    } else {
        LFQ_TRY(grow(&S->d_in, &S->d_in_bytes, lfq_al(rec_bytes + 16)));
        const uint8_t *src = body + first;
        if (!lfq_is_pinned(src)) {
            if (rec_bytes > S->h_stage_bytes) {
                LFQ_TRY(grow_pinned(&S->h_stage, &S->h_stage_bytes, std::max<int64_t>(rec_bytes + rec_bytes / 4, 1 << 16)));
            }
            memcpy(S->h_stage, src, (size_t)rec_bytes);
            src = S->h_stage;
        }
        LFQ_TRY_HIP(hipMemcpyAsync(S->d_in, src, (size_t)rec_bytes, hipMemcpyHostToDevice, st));
        d_recs = S->d_in;
    }
    LFQ_TRY_HIP(hipMemcpyAsync(S->d_buf, tab.data(), (size_t)(n_recs + 1) * 8, hipMemcpyHostToDevice, st));
    LFQ_TRY_HIP(hipMemcpyAsync(S->d_buf + o_doff, tab.data() + n_recs + 1, (size_t)(n_blocks + 1) * 8, hipMemcpyHostToDevice, st));
    LFQ_TRY_HIP(hipMemcpyAsync(S->d_buf + o_coff, tab.data() + n_recs + 1 + n_blocks + 1, (size_t)(n_blocks + 1) * 8,
                               hipMemcpyHostToDevice, st));
    LFQ_TRY_HIP(hipMemcpyAsync(dev.counters, cnt.data(), 32, hipMemcpyHostToDevice, st));
    LFQ_TRY(S->up_t.end(st));
    LfqBaiArgs A = S->lay;
    A.body = d_recs - first;            /* (never read in front of rec_off[0]) */
    A.rec_off = (const int64_t *)S->d_buf;
    A.data_off = (const int64_t *)(S->d_buf + o_doff);
    A.comp_off = (const int64_t *)(S->d_buf + o_coff);
    A.n_blocks = n_blocks;
    A.file_off = file_off;
    A.n_ref = n_ref;
    const dim3 grid((unsigned)A.n_parts), block(LFQ_BAI_THREADS);
    LFQ_TRY(S->kern_t.begin(st));
    hipLaunchKernelGGL(lfq_bai_record_kernel, grid, block, 0, st, A);
    LFQ_TRY_HIP(hipGetLastError());
    LFQ_TRY(S->kern_t.end(st));
    S->times.n_launches = 1;
    /* the first refused record, before the lists are made of records that may not be sorted */
    LFQ_TRY(S->down_t.begin(st));
    LFQ_TRY_HIP(hipMemcpyAsync(cnt.data(), A.counters, 8, hipMemcpyDeviceToHost, st));
    LFQ_TRY(S->down_t.end(st));
    LFQ_TRY_HIP(hipStreamSynchronize(st));
    LFQ_TRY(bam_idx_add_ms(S->up_t, &S->times.upload_ms));
    LFQ_TRY(bam_idx_add_ms(S->kern_t, &S->times.kernels_ms));
    LFQ_TRY(bam_idx_add_ms(S->down_t, &S->times.download_ms));
    if (cnt[0] != ~0ull) {
        S->times.first_bad_record = (int64_t)cnt[0];
        return LFQ_ERR_INVALID;
    }
    LfqBaiLists L;
    LFQ_TRY(lfq_bai_compact(c, &L));
    S->times.n_launches = 4;
    S->times.kernels_ms += L.kernels_ms;
    S->times.download_ms += L.download_ms;
    const int64_t n_chunks = L.n_chunks, n_intvs = L.n_intvs;
    S->times.n_chunks = n_chunks;
    S->times.n_intervals = n_intvs;
    const auto t0 = std::chrono::steady_clock::now();
    if (!lfq_bai_finish(L.chunks, n_chunks, L.runs, L.n_runs, L.intvs, n_intvs, n_ref, n_recs, idx)) {
        return LFQ_ERR_HIP;
    }
    S->times.host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    drop.p = nullptr;
    *out = idx;
    return LFQ_OK;
}

extern "C" int lfq_last_bam_index_times(lfq_ctx *c, lfq_bam_index_times *t)
{
    if (!c || !t) {
        return LFQ_ERR_INVALID;
    }
    *t = bam_idx_state(c)->times;
    return LFQ_OK;
}

/* ---- host only: no context ------------------------------------------------------------------------------------------------------------ */
extern "C" int lfq_bam_index_bytes(const lfq_bam_index *idx, const uint8_t **bai, int64_t *n_bytes)
{
    if (!idx || !bai || !n_bytes) {
        return LFQ_ERR_INVALID;
    }
    lfq_bam_index *m = const_cast<lfq_bam_index *>(idx);        /* (the cache of the serialised form is not part of its value) */
    if (m->bytes.empty()) {
        lfq_bai_serialise(*m, &m->bytes);
    }
    *bai = m->bytes.data();
    *n_bytes = (int64_t)m->bytes.size();
    return LFQ_OK;
}

extern "C" int lfq_bam_index_parse(const uint8_t *bai, int64_t n_bytes, lfq_bam_index **out)
{
    if (out) *out = nullptr;
    if (!bai || !out || n_bytes < 0) {
        return LFQ_ERR_INVALID;
    }
    lfq_bam_index *idx = new lfq_bam_index();
    if (!lfq_bai_parse(bai, n_bytes, idx)) {
        delete idx;
        return LFQ_ERR_INVALID;
    }
    *out = idx;
    return LFQ_OK;
}

extern "C" int lfq_bam_index_query(const lfq_bam_index *idx, int32_t tid, int64_t beg, int64_t end, const uint64_t **chunk_beg,
                                   const uint64_t **chunk_end, int64_t *n_chunks)
{
    if (!idx || !chunk_beg || !chunk_end || !n_chunks || tid < 0 || (size_t)tid >= idx->refs.size()) {
        return LFQ_ERR_INVALID;
    }
    lfq_bam_index *m = const_cast<lfq_bam_index *>(idx);        /* (the result's storage) */
    lfq_bai_query(m, tid, beg, end);
    *chunk_beg = m->q_beg.data();
    *chunk_end = m->q_end.data();
    *n_chunks = (int64_t)m->q_beg.size();
    return LFQ_OK;
}

extern "C" void lfq_bam_index_free(lfq_bam_index *idx) { delete idx; }

extern "C" int lfq_bam_record_chain(const uint8_t *bam, int64_t first, int64_t stop, int64_t **rec_off, int64_t *n_recs)
{
    if (rec_off) *rec_off = nullptr;
    if (!bam || !rec_off || !n_recs || first < 0 || stop < first) {
        return LFQ_ERR_INVALID;
    }
    std::vector<int64_t> off(1, first);
    while (off.back() + 4 <= stop) {
        const int64_t size = (int32_t)lfq_bai_ld32(bam + off.back());
        if (size < 32) {
            return LFQ_ERR_INVALID;
        }
        if (off.back() + 4 + size > stop) {
            break;
        }
        off.push_back(off.back() + 4 + size);
    }
    int64_t *p = (int64_t *)malloc(off.size() * sizeof(int64_t));
    if (!p) {
        return LFQ_ERR_NOMEM;
    }
    memcpy(p, off.data(), off.size() * sizeof(int64_t));
    *rec_off = p;
    *n_recs = (int64_t)off.size() - 1;
    return LFQ_OK;
}

extern "C" void lfq_bam_record_chain_free(int64_t *rec_off) { free(rec_off); }

extern "C" int lfq_bam_record_cuts(const int64_t *rec_off, int64_t n_recs, int64_t max_piece, int64_t **cuts, int64_t *n_cuts)
{
    if (cuts) *cuts = nullptr;
    if (!rec_off || !cuts || !n_cuts || n_recs < 0 || max_piece <= 0) {
        return LFQ_ERR_INVALID;
    }
    for (int64_t j = 0; j < n_recs; j++) {
        if (rec_off[j + 1] <= rec_off[j]) {
            return LFQ_ERR_INVALID;
        }
    }
    std::vector<int64_t> out;
    int64_t start = rec_off[0], j = 1;
    while (rec_off[n_recs] - start > max_piece) {
        while (j <= n_recs && rec_off[j] - start <= max_piece) {
            j++;
        }
        const int64_t cut = rec_off[j - 1] > start ? rec_off[j - 1] : start + max_piece;
        out.push_back(cut);
        start = cut;
    }
    int64_t *p = (int64_t *)malloc(std::max<size_t>(out.size(), 1) * sizeof(int64_t));
    if (!p) {
        return LFQ_ERR_NOMEM;
    }
    memcpy(p, out.data(), out.size() * sizeof(int64_t));
    *cuts = p;
    *n_cuts = (int64_t)out.size();
    return LFQ_OK;
}

extern "C" void lfq_bam_record_cuts_free(int64_t *cuts) { free(cuts); }
